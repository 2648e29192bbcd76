"""Estimates from a saved SVR or KNR model on the GPU (csrc/kpredict.hip): the "file route" the offloading
cascade is held to for these two kinds.

    model = kpredict.load("wts1.pickle")        # or the dict edgeml_amd.svr / regress.model_data returns
    est = model.to("cuda").predict(features)    # float64 [N], in chunks of any size

An SVR file holds {model, mean, scale, gamma, support (raw feature rows), beta, intercept}; a KNR file {model,
mean, scale, n_neighbors, train (raw training rows, training-list order), target}.  to() uploads the arrays and
standardises the stored rows once (edgedet_kmodel_prepare, in the fits' own order); predict() standardises the
queries in the load.  Float64 throughout; an estimate depends on the feature row and the model only, not on
the chunk it was computed in, and a KNR model reproduces edgeml_amd.regress.fit_knr's estimates and neighbours
bit for bit.  There is no CPU path.
"""
import pickle

import numpy as np
import torch

from . import ops

KINDS = {"SVR": 0, "KNR": 1}
CHUNK = 4096  # rows per predict call: bounds the KNR distance workspace (8 n bytes a row)


def _need_device():
    if not torch.cuda.is_available():
        raise RuntimeError("edgeml_amd.kpredict needs an MI355X (HIP) device; there is no CPU path")


def _vec(what, m, key, n=None):
    if key not in m:
        raise ValueError(f"{what}: no '{key}'")
    a = np.ascontiguousarray(np.asarray(m[key], np.float64).reshape(-1))
    if n is not None and len(a) != n:
        raise ValueError(f"{what}: '{key}' has {len(a)} entries, expected {n}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: '{key}' is not finite")
    return a


def _rows(what, m, key, D):
    a = np.asarray(m[key], np.float64)
    if a.ndim != 2 or a.shape[1] != D:
        raise ValueError(f"{what}: '{key}' has shape {a.shape}, expected [rows][{D}] as mean and scale are {D} wide")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: '{key}' is not finite")
    return np.ascontiguousarray(a)


def _scalar(what, m, key):
    if key not in m:
        raise ValueError(f"{what}: no '{key}'")
    v = float(m[key])
    if not np.isfinite(v):
        raise ValueError(f"{what}: '{key}' is not finite")
    return v


class KernelModel:
    """kind "svr": rows = the support vectors, weight = beta, gamma, intercept; kind "knr": rows = the training
    rows, weight = their targets, n_neighbors.  mean, scale [width] are the fold's StandardScaler."""

    def __init__(self, kind, mean, scale, rows, weight, gamma=0.0, intercept=0.0, n_neighbors=0):
        self.kind, self.width, self.n = kind, len(mean), len(rows)
        self.mean, self.scale, self.rows, self.weight = mean, scale, rows, weight
        self.gamma, self.intercept, self.n_neighbors = float(gamma), float(intercept), int(n_neighbors)
        self._dev = None

    # ------------------------------------------------------------------------------------ device side
    def to(self, device):
        """Upload and prepare once per device; returns self."""
        _need_device()
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if self._dev is not None and self._dev["device"] == device:
            return self
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        d = {"device": device, "mean": t(self.mean), "scale": t(self.scale), "weight": t(self.weight),
             "z": torch.empty((self.n, self.width), dtype=torch.float64, device=device),
             "norm": torch.empty((self.n,), dtype=torch.float64, device=device)}
        rows = t(self.rows)
        p = ops._ptr
        with torch.cuda.device(device):
            ops.check(ops.lib().edgedet_kmodel_prepare(p(rows), self.n, self.width, p(d["mean"]), p(d["scale"]),
                                                       p(d["z"]), p(d["norm"]), ops.stream_handle()))
            torch.cuda.current_stream().synchronize()  # rows may be freed; other streams may read z
        self._dev = d
        return self

    def workspace_bytes(self, B):
        wb = int(ops.lib().edgedet_kmodel_workspace_size(self.n, self.width, int(B), KINDS[self.kind.upper()]))
        if wb < 0:
            raise ValueError(f"edgeml_amd.kpredict: no workspace for {B} rows of {self.width} features against "
                             f"{self.n} stored rows")
        return wb

    def predict_into(self, feat, est, ws, nbr=None, stream=None):
        """One library call: feat [B, width] float64 and est [B] float64 on the prepared device, ws a uint8
        tensor of workspace_bytes(B); nbr [B, n_neighbors] int32 receives a KNR model's neighbours."""
        d = self._dev
        if d is None or d["device"] != feat.device:
            raise ValueError("edgeml_amd.kpredict: call to(device) with the features' device first")
        ops._need_cuda(feat, est, ws, nbr)
        B, p, L = int(feat.shape[0]), ops._ptr, ops.lib()
        if feat.dtype != torch.float64 or feat.dim() != 2 or feat.shape[1] != self.width or est.dtype != torch.float64 \
                or est.numel() < B:
            raise ValueError(f"edgeml_amd.kpredict: features [B][{self.width}] and estimates [B] in float64")
        if self.kind == "svr":
            ops.check(L.edgedet_svr_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]), p(d["z"]),
                                                  p(d["norm"]), p(d["weight"]), self.n, self.gamma, self.intercept,
                                                  p(ws), ws.numel(), p(est), ops.stream_handle(stream)))
        else:
            if nbr is not None and (nbr.dtype != torch.int32 or nbr.numel() < B * self.n_neighbors):
                raise ValueError("edgeml_amd.kpredict: neighbours [B][n_neighbors] in int32")
            ops.check(L.edgedet_knn_model_predict(p(feat), B, self.width, p(d["mean"]), p(d["scale"]), p(d["z"]),
                                                  p(d["norm"]), p(d["weight"]), self.n, self.n_neighbors, p(ws),
                                                  ws.numel(), p(est), p(nbr), ops.stream_handle(stream)))

    def predict(self, features, chunk=CHUNK, neighbors=False):
        """Estimates float64 [N] of features [N, ...] (flattened to [N, width]); with neighbors=True a KNR
        model also returns the neighbours' positions int32 [N, n_neighbors], ascending."""
        _need_device()
        if self._dev is None:
            self.to("cuda")
        dev = self._dev["device"]
        x = np.asarray(features, dtype=np.float64)
        x = np.ascontiguousarray(x.reshape(len(x), -1))
        if x.shape[1] != self.width:
            raise ValueError(f"edgeml_amd.kpredict: the model takes {self.width} features, the rows have {x.shape[1]}")
        if neighbors and self.kind != "knr":
            raise ValueError("edgeml_amd.kpredict: only a KNR model has neighbours")
        chunk = max(1, int(chunk))
        N, k = len(x), self.n_neighbors
        est = np.empty(N, np.float64)
        nbr = np.empty((N, k), np.int32) if neighbors else None
        if N == 0:
            return (est, nbr) if neighbors else est
        with torch.cuda.device(dev):
            ws = torch.empty(self.workspace_bytes(min(chunk, N)), dtype=torch.uint8, device=dev)
            g_est = torch.empty(min(chunk, N), dtype=torch.float64, device=dev)
            g_nbr = torch.empty((min(chunk, N), k), dtype=torch.int32, device=dev) if neighbors else None
            for a in range(0, N, chunk):
                b = min(a + chunk, N)
                self.predict_into(torch.from_numpy(x[a:b]).to(dev), g_est, ws, g_nbr)
                est[a:b] = g_est[:b - a].cpu().numpy()
                if neighbors:
                    nbr[a:b] = g_nbr[:b - a].cpu().numpy()
        return (est, nbr) if neighbors else est


def load(path_or_dict):
    """The KernelModel of an SVR or KNR wts<fold>.pickle (a path, or the dict itself); ValueError on anything
    else, on inconsistent shapes and on values that are not finite."""
    if isinstance(path_or_dict, dict):
        m, what = path_or_dict, "model"
    else:
        what = str(path_or_dict)
        with open(path_or_dict, "rb") as f:
            m = pickle.load(f)
    if not isinstance(m, dict) or "mean" not in m or "scale" not in m:
        raise ValueError(f"{what}: not a wts<fold>.pickle of edgeml_amd.estimator / edgeml_amd.svr --model-dir")
    mean = _vec(what, m, "mean")
    D = len(mean)
    scale = _vec(what, m, "scale", D)
    if not 1 <= D <= 255:
        raise ValueError(f"{what}: {D} features; the kernels take 1 to 255")
    if np.any(scale == 0.0):
        raise ValueError(f"{what}: a zero in 'scale'")
    kind = m.get("model")
    if kind == "SVR":
        if "support" not in m or "beta" not in m:
            raise ValueError(f"{what}: an SVR file without 'support' and 'beta'")
        support = _rows(what, m, "support", D)
        beta = _vec(what, m, "beta", len(support))
        gamma = _scalar(what, m, "gamma")
        if gamma <= 0.0:
            raise ValueError(f"{what}: gamma = {gamma!r} is not positive")
        return KernelModel("svr", mean, scale, support, beta, gamma=gamma, intercept=_scalar(what, m, "intercept"))
    if kind == "KNR":
        if "train" not in m or "target" not in m:
            raise ValueError(f"{what}: a KNR file holds no training rows (written before --model-dir stored them): "
                             f"train it again")
        train = _rows(what, m, "train", D)
        target = _vec(what, m, "target", len(train))
        kn, n = int(_scalar(what, m, "n_neighbors")), len(train)
        if kn > n:  # sklearn's wording (neighbors/_base.py kneighbors), as regress.fit_knr uses it
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {kn}, n_samples_fit = {n}, "
                             f"n_samples = {n}")
        if kn < 1:
            raise ValueError(f"Expected n_neighbors > 0. Got {kn}")
        return KernelModel("knr", mean, scale, train, target, n_neighbors=kn)
    raise ValueError(f"{what}: model {kind!r} is neither SVR nor KNR (a linear or CNN file predicts through "
                     f"edgeml_amd.offload.load_estimator)")
